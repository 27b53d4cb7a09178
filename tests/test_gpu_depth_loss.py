"""GPU (-m gpu): gs_depth_loss_forward / gs_depth_loss_backward (include/gs_depth.h) through depth.py, all 16 flag
combinations, against the float64 restatement tests/depth_ref.evaluate.

Sizes: 1x1, 3x5, 17x61 (odd width: the pixel-by-pixel path and a ragged last thread), 64x96, and 520x512 = 260 blocks of 1024
pixels: more than one block and more than the 256 threads of a finishing block, so both of its loops run.

Bars: four times the error of the same formulas in torch float32 on the CPU (depth_ref.evaluate(dtype=float32)) against the
reference, measured inside the test, with one f32 ulp of the value as the floor -- the precedent of the mixture gradient tests.
For a gradient "the value" is the largest magnitude of the plane.  The number of selected pixels and every unselected
gradient (+0) are exact.  L1 gradient: a pixel whose |r_ref| is below 1e-6 of the largest |r_ref| may have either sign and is
left out; at most 0.1 % of the pixels may be (the random continuous inputs stay far below that).  The 1x1 case uses values that
are exact in f32, so that its single pixel does not make the measured f32 error an accident."""
import functools

import numpy as np
import pytest
import torch

import depth_ref as R
from taichi_3d_gaussian_splatting_amd import depth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(1, 1), (3, 5), (17, 61), (64, 96), (520, 512)]
ALL_FLAGS = list(range(16))


def ulp(value):
    return float(np.spacing(np.float32(abs(float(value)))))


@functools.lru_cache(maxsize=None)
def planes(h, w, seed=0):
    """D, Z, w_t, w_p on the CPU: about half the pixels selected; empty pixels (D = 0), holes (w_t = 0) and masked pixels"""
    if (h, w) == (1, 1):
        return torch.tensor([[2.0]]), torch.tensor([[4.0]]), torch.tensor([[0.5]]), torch.tensor([[0.25]])
    g = torch.Generator().manual_seed(1000 * h + w + seed)
    Z = 1.0 + 4.0 * torch.rand(h, w, generator=g)
    D = Z * (1.0 + 0.3 * (torch.rand(h, w, generator=g) - 0.5))
    w_t = 0.05 + 0.95 * torch.rand(h, w, generator=g)
    w_p = 0.05 + 0.95 * torch.rand(h, w, generator=g)
    w_t[torch.rand(h, w, generator=g) < 0.3] = 0.0
    w_p[torch.rand(h, w, generator=g) < 0.15] = 0.0
    D[torch.rand(h, w, generator=g) < 0.1] = 0.0
    if h * w >= 15:
        w_t[0, 0], D[0, 1], w_t[-1, -1] = 0.8, 0.0, 0.6          # the first pixel selected, the second empty, the last selected
        D[0, 0], D[-1, -1] = 2.0, 3.0
        w_p[0, 0] = w_p[-1, -1] = 0.9
    return D, Z, w_t, w_p


def dev(*tensors):
    return tuple(None if t is None else t.to(DEV).contiguous() for t in tensors)


def run(D, Z, w_t, w_p, flags, upstream=None):
    """-> (terms (8,), grad (H,W)) on the CPU from the library, twice: the same bits"""
    d = dev(D, Z, w_t, w_p)
    up = None if upstream is None else torch.tensor([upstream], dtype=torch.float32, device=DEV)
    terms = depth.depth_loss_forward(*d, flags=flags)
    grad = depth.depth_loss_backward(*d, flags, terms, upstream=up)
    terms2 = depth.depth_loss_forward(*d, flags=flags)
    grad2 = depth.depth_loss_backward(*d, flags, terms2, upstream=up)
    assert torch.equal(terms.view(torch.int32), terms2.view(torch.int32)) and torch.equal(grad.view(torch.int32), grad2.view(torch.int32))
    return terms.cpu(), grad.cpu()


def compare(D, Z, w_t, w_p, flags, upstream=None, label=""):
    u = 1.0 if upstream is None else upstream
    ref = R.evaluate(D, Z, w_t, w_p, flags, upstream=u)
    f32 = R.evaluate(D, Z, w_t, w_p, flags, upstream=u, dtype=torch.float32)
    terms, grad = run(D, Z, w_t, w_p, flags, upstream)
    assert torch.isfinite(terms).all() and torch.isfinite(grad).all()
    for k, name in enumerate(("L", "S_w", "s", "t")):
        want = ref["terms"][k].item()
        bar = max(4 * abs(f32["terms"][k].item() - want), ulp(want))
        err = abs(terms[k].item() - want)
        print(f"{label} flags {flags:2d} {name}: error {err:.3g} bar {bar:.3g}")
        assert err <= bar, (name, err, bar)
    assert terms[4].item() == ref["terms"][4].item() and not terms[5:].any()
    off = ~ref["selected"]
    assert not grad[off].any() and not torch.signbit(grad[off]).any()             # exactly +0
    keep = ref["selected"].clone()
    if not flags & R.L2 and bool(keep.any()):
        near = ref["selected"] & (ref["r"].abs() < 1e-6 * ref["r"].abs().max())
        assert near.double().mean().item() <= 0.001
        keep &= ~near
    if bool(keep.any()):
        want = ref["grad"][keep]
        bar = max(4 * (f32["grad"][keep].double() - want).abs().max().item(), ulp(want.abs().max().item()))
        err = (grad[keep].double() - want).abs().max().item()
        print(f"{label} flags {flags:2d} grad: error {err:.3g} bar {bar:.3g}")
        assert err <= bar, (err, bar)
    return terms, grad


@pytest.mark.parametrize("flags", ALL_FLAGS)
@pytest.mark.parametrize("h,w", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_all_flags_against_the_reference(h, w, flags):
    D, Z, w_t, w_p = planes(h, w)
    compare(D, Z, w_t, w_p, flags, label=f"{h}x{w}")


@pytest.mark.parametrize("flags", [0, 3, 7, 9, 12, 15])
def test_one_weight_plane_and_a_device_upstream(flags):
    D, Z, w_t, w_p = planes(17, 61)
    with_both, _ = compare(D, Z, w_t, w_p, flags)
    with_one, _ = compare(D, Z, w_t, None, flags)
    assert with_one[4].item() > with_both[4].item()                    # the second plane masks pixels the first keeps
    _, g1 = compare(D, Z, w_t, w_p, flags, upstream=1.0)
    _, g = compare(D, Z, w_t, w_p, flags, upstream=-0.37)
    assert g.abs().max() > 0 and not torch.equal(g, g1)


@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_an_empty_selection_gives_zeros(flags):
    D, Z, w_t, w_p = planes(17, 61)
    for args in ((D, Z, torch.zeros_like(w_t), w_p), (torch.zeros_like(D), Z, w_t, None), (D, torch.full_like(Z, float("nan")), w_t, w_p),
                 (D, Z, w_t, torch.full_like(w_p, -1.0))):
        terms, grad = run(*args, flags)
        assert not terms.any() and not torch.signbit(terms).any()
        assert not grad.any() and not torch.signbit(grad).any()


@pytest.mark.parametrize("flags", [8, 9, 11, 12, 15])
def test_degenerate_fits(flags):
    D, Z, w_t, w_p = planes(17, 61)
    one = torch.zeros_like(w_t)
    one[5, 7] = 0.7
    D1 = D.clone()
    D1[5, 7] = 2.5
    terms, grad = compare(D1, Z, one, None, flags)                        # a single pixel: s = 0, t = x, no residual
    x = 1.0 / 2.5 if flags & R.INVERT_PREDICTED else 2.5
    assert terms[2].item() == 0.0 and abs(terms[3].item() - x) <= ulp(x) and terms[0].item() <= ulp(x) and terms[4].item() == 1.0
    constant = torch.full_like(Z, 2.0)
    terms, _ = compare(D, constant, w_t, w_p, flags)                      # a constant target: s = 0, t = the weighted mean of x
    assert terms[2].item() == 0.0 and terms[3].item() > 0.0


def test_unusable_values_under_a_zero_weight_are_inert():
    D, Z, w_t, w_p = planes(64, 96)
    for flags in (0, 6, 9, 15):
        ref = R.evaluate(D, Z, w_t, w_p, flags)
        terms, grad = compare(D, Z, w_t, w_p, flags)
        off = ~ref["selected"]
        bad = torch.tensor([float("nan"), float("inf"), -float("inf"), -3.0, 0.0, -0.0])
        fill = bad[torch.arange(int(off.sum())) % len(bad)]
        D2, Z2, wt2, wp2 = D.clone(), Z.clone(), w_t.clone(), w_p.clone()
        # each unselected pixel keeps one reason not to be selected and gets unusable values everywhere else
        zero_wt = off & (w_t == 0)
        zero_wp = off & (w_p == 0) & ~zero_wt
        zero_D = off & ~zero_wt & ~zero_wp
        D2[zero_wt | zero_wp] = fill[: int((zero_wt | zero_wp).sum())]
        Z2[off] = fill.flip(0)
        wp2[zero_wt] = float("inf")                                      # inf * 0 is NaN, not a weight
        wt2[zero_wp] = float("inf")
        wt2[zero_D & (torch.arange(D.numel()).reshape(D.shape) % 2 == 0)] = float("nan")      # a NaN weight counts as 0
        wp2[zero_D & (torch.arange(D.numel()).reshape(D.shape) % 3 == 0)] = -2.0              # so does a negative one
        terms2, grad2 = run(D2, Z2, wt2, wp2, flags)
        assert torch.equal(terms.view(torch.int32), terms2.view(torch.int32)) and torch.equal(grad.view(torch.int32), grad2.view(torch.int32))


@pytest.mark.parametrize("h,w", [(17, 61), (64, 96)])
def test_aligned_and_misaligned_planes_give_equal_bits(h, w):
    D, Z, w_t, w_p = planes(h, w)
    n = h * w

    def shifted(t, k):
        """the plane at an offset of k floats behind a 16-byte aligned base"""
        buf = torch.zeros(n + 8, dtype=torch.float32, device=DEV)
        assert buf.data_ptr() % 16 == 0
        view = buf[k:k + n].view(h, w)
        view.copy_(t)
        return view

    for flags in (0, 7, 9, 15):
        results = []
        for offsets in ((0, 0, 0, 0, 0), (1, 1, 1, 1, 1), (0, 1, 2, 3, 1), (3, 0, 0, 1, 0)):
            d, z, a, b = (shifted(t, k) for t, k in zip((D, Z, w_t, w_p), offsets))
            out = shifted(torch.zeros(h, w), offsets[4])
            terms = depth.depth_loss_forward(d, z, a, b, flags=flags)
            depth.depth_loss_backward(d, z, a, b, flags, terms, out=out)
            results.append((terms.cpu(), out.cpu()))
        for terms, grad in results[1:]:
            assert torch.equal(terms.view(torch.int32), results[0][0].view(torch.int32))
            assert torch.equal(grad.view(torch.int32), results[0][1].view(torch.int32))


def test_a_planted_scale_and_shift_come_back_in_the_terms():
    """a monocular prior y = a / Z_true + b against the rendering x = 1 / Z_true: s = 1 / a, t = -b / a"""
    _, Z_true, w_t, w_p = planes(64, 96)
    a, b = 2.5, 0.3
    prior = a / Z_true + b
    flags = depth.loss_flags("inverse", "l1", align=True, target_is_inverse=True)
    assert flags == R.INVERT_PREDICTED | R.ALIGN
    terms = depth.depth_loss_forward(*dev(Z_true, prior, w_t, w_p), flags=flags).cpu()
    assert abs(terms[2].item() - 1 / a) < 1e-5 and abs(terms[3].item() + b / a) < 1e-5 and terms[0].item() < 1e-6
    loss = depth.depth_loss(*dev(Z_true, prior, w_t, w_p), space="inverse", norm="l1", align=True, target_is_inverse=True)
    assert torch.equal(loss.terms.cpu(), terms) and loss.item() == terms[0].item()


@pytest.mark.parametrize("flags", [12, 13, 15])
def test_envelope_the_l2_aligned_gradient_is_the_total_derivative(flags):
    D, Z, w_t, w_p = planes(17, 61)
    Dd = D.double().requires_grad_(True)
    R.loss_through_fit(Dd, Z, w_t, w_p, flags).backward()              # float64, the fit NOT detached
    want = Dd.grad
    f32 = R.evaluate(D, Z, w_t, w_p, flags, dtype=torch.float32)["grad"].double()
    _, grad = run(D, Z, w_t, w_p, flags)
    bar = max(4 * (f32 - want).abs().max().item(), ulp(want.abs().max().item()))
    err = (grad.double() - want).abs().max().item()
    print(f"flags {flags}: error {err:.3g} bar {bar:.3g}")
    assert err <= bar


def test_autograd_reaches_depth_only_and_keeps_the_terms():
    D, Z, w_t, w_p = dev(*planes(64, 96))
    D.requires_grad_(True)
    loss = depth.depth_loss(D, Z, w_t, w_p, space="inverse", norm="l2", align=True)
    assert loss.dim() == 0 and loss.terms.shape == (8,) and not loss.terms.requires_grad
    (0.25 * loss).backward()
    flags = depth.loss_flags("inverse", "l2", True)
    want = depth.depth_loss_backward(D.detach(), Z, w_t, w_p, flags, loss.terms, upstream=torch.tensor([0.25], device=DEV))
    assert torch.equal(D.grad, want) and D.grad.abs().max() > 0
