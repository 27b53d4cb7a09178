"""CPU: the numpy restatement of include/gs_background.h (background_ref.py) against its own float64 closed form and against
torch float64 autograd of x + (1 - A) c.  This pins the yardstick of the GPU tests."""
import numpy as np
import pytest
import torch

import background_ref as ref

H, W = 37, 29                                  # 1073 pixels: two blocks of the backward, W % 4 != 0


def _case(seed, h=H, w=W):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 1.0, (3, h, w)).astype(np.float32)
    A = rng.uniform(0.0, 1.0, (h, w)).astype(np.float32)
    g = rng.normal(0.0, 1.0, (3, h, w)).astype(np.float32)
    coef = rng.normal(0.0, 0.5, 48).astype(np.float32)
    q = rng.normal(0.0, 1.0, 4).astype(np.float32)
    q = (q / np.linalg.norm(q) * 1.3).astype(np.float32)          # not a unit quaternion: it is used as it is
    K9 = ref.camera(h, w, fx=0.9 * w, fy=1.1 * w, cx=0.4 * w, cy=0.55 * h)
    return x, A, g, coef, q, K9


@pytest.mark.parametrize("bands", [0, 1, 2, 3])
@pytest.mark.parametrize("flags", [0, ref.STRAIGHT, ref.COLOURS_ONLY])
def test_forward_agrees_with_the_float64_closed_form(bands, flags):
    """Bound: the direction takes about 8 f32 roundings (5e-7 relative), a basis value is a polynomial of degree <= 3 whose
    gradient is below 7 and takes up to 6 more (4e-6 absolute in all), and the K-term sum adds K eps of the terms' magnitudes:
    1e-5 (|x| + sum_k |coef_k| (|Y_k| + 1)), twice the estimate.  |q| = 1.3 scales R, so a basis value is below 4 * 1.3^3 < 9."""
    x, A, g, coef, q, K9 = _case(bands)
    first = (H, W) if flags & ref.COLOURS_ONLY else x
    got = ref.composite(first, A, coef, bands, q, K9, flags)
    want = ref.composite(first, A, coef, bands, q, K9, flags, dtype=np.float64)
    assert got.dtype == np.float32 and want.dtype == np.float64 and got.shape == (3, H, W)
    Y = np.abs(ref._basis_np(bands, q, K9, H, W, np.float64))
    assert Y.max() < 9.0
    Kn = (bands + 1) ** 2
    bound = np.stack([sum(abs(float(coef[16 * i + k])) * (Y[k] + 1.0) for k in range(Kn)) for i in range(3)]) + 1.0
    err = np.abs(got - want)
    print(f"bands {bands} flags {flags}: max error {err.max():.3e}, largest error / bound {float((err / (1e-5 * bound)).max()):.3f}")
    assert np.all(err <= 1e-5 * bound)


def _torch_gradients(x, A, g, coef, bands, q, K9, dtype):
    """autograd of sum g (x + (1 - A) c) in `dtype`, the basis by the same formulas in torch -> (grad_alpha, grad_coef)"""
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    At, ct = t(A).requires_grad_(True), t(coef).requires_grad_(True)
    py, px = torch.meshgrid(torch.arange(A.shape[0], dtype=dtype), torch.arange(A.shape[1], dtype=dtype), indexing="ij")
    Y = ref.basis(px, py, t(q), t(K9).reshape(9), c=float, sqrt=torch.sqrt) if bands > 0 else [1.0] * 16
    c = ref.colour(ct, Y, bands)
    out = torch.stack([t(x)[i] + (1.0 - At) * c[i] for i in range(3)])
    out.backward(t(g))
    return At.grad.numpy(), ct.grad.numpy()


@pytest.mark.parametrize("bands", [0, 1, 2, 3])
def test_gradients_agree_with_float64_autograd(bands):
    """The bar of the mixture-gradient tests: the restatement may be off float64 autograd by 4 x what the same formulas in
    torch float32 on the CPU are off by."""
    x, A, g, coef, q, K9 = _case(10 + bands)
    g[:, 2, 3] = 0.0                                    # one pixel that is not selected
    ga64, gc64 = _torch_gradients(x, A, g, coef, bands, q, K9, torch.float64)
    ga32, gc32 = _torch_gradients(x, A, g, coef, bands, q, K9, torch.float32)
    ga, gc = ref.grad_alpha(g, coef, bands, q, K9), ref.grad_coef(g, A, bands, q, K9)
    assert ga.dtype == np.float32 and gc.dtype == np.float32 and ga.shape == (H, W) and gc.shape == (48,)
    for name, got, torch32, want in (("grad_alpha", ga, ga32, ga64), ("grad_coef", gc, gc32, gc64)):
        mine, theirs = float(np.abs(got - want).max()), float(np.abs(torch32 - want).max())
        print(f"bands {bands} {name}: restatement {mine:.3e}, torch float32 {theirs:.3e} off float64 autograd")
        assert theirs > 0.0
        assert mine <= 4.0 * theirs, name
    assert ga[2, 3] == 0.0 and not np.signbit(ga[2, 3])
    Kn = (bands + 1) ** 2
    for i in range(3):
        assert np.all(gc[16 * i + Kn:16 * i + 16] == 0.0) and np.all(gc[16 * i:16 * i + Kn] != 0.0)
    # the closed form of the restatement itself is that autograd
    assert np.abs(ref.grad_coef(g, A, bands, q, K9, dtype=np.float64) - gc64).max() <= 1e-12 * ref.grad_coef_magnitude(g, A, bands, q, K9).max()
    assert np.abs(ref.grad_alpha(g, coef, bands, q, K9, dtype=np.float64) - ga64).max() <= 1e-13


@pytest.mark.parametrize("bands", [0, 1, 2, 3])
def test_white_over_nothing_is_exactly_one_and_full_alpha_keeps_the_image(bands):
    x, A, g, coef, q, K9 = _case(20 + bands)
    out = ref.composite(np.zeros_like(x), np.zeros_like(A), ref.WHITE, bands, q, K9)
    assert np.all(out == np.float32(1.0))
    assert np.all(ref.colours(ref.WHITE, bands, q, K9, H, W) == np.float32(1.0))
    out = ref.composite(x, np.ones_like(A), coef, bands, q, K9)
    assert out.tobytes() == x.tobytes()
    # straight alpha 1 as well: x * 1 + 0 * c
    assert ref.composite(x, np.ones_like(A), coef, bands, q, K9, ref.STRAIGHT).tobytes() == x.tobytes()


def test_a_solid_colour_ignores_the_camera():
    x, A, g, coef, q, K9 = _case(30)
    a = ref.composite(x, A, coef, 0, q, K9)
    b = ref.composite(x, A, coef, 0, None, None)
    c = ref.composite(x, A, coef, 0, -q[::-1].copy(), ref.camera(H, W))
    assert a.tobytes() == b.tobytes() == c.tobytes()
    assert ref.grad_coef(g, A, 0, q, K9).tobytes() == ref.grad_coef(g, A, 0).tobytes()
    assert ref.grad_alpha(g, coef, 0, q, K9).tobytes() == ref.grad_alpha(g, coef, 0).tobytes()
    assert np.all(a == x + (np.float32(1.0) - A) * coef[[0, 16, 32]][:, None, None])


def test_half_a_turn_about_the_optical_axis_flips_y1_and_y3():
    """a centred camera: the pixel mirrored through the centre looks along (-a, -b, 1), which is what a rotation of the camera
    by 180 degrees about its optical axis turns (a, b, 1) into.  Y_1 ~ y and Y_3 ~ x change sign, Y_2 ~ z does not -- exactly."""
    h, w = 6, 8
    K9 = ref.camera(h, w)
    coef = np.zeros(48, dtype=np.float32)
    coef[1], coef[16 + 2], coef[32 + 3] = 1.0, 1.0, 1.0          # channel 0 shows Y_1, channel 1 Y_2, channel 2 Y_3
    identity = np.array([0, 0, 0, 1], dtype=np.float32)
    turned = np.array([0, 0, 1, 0], dtype=np.float32)
    a = ref.colours(coef, 1, identity, K9, h, w)
    b = ref.colours(coef, 1, turned, K9, h, w)
    assert np.all(a[0] != 0.0) and np.all(a[2] != 0.0)
    assert np.array_equal(b[0], -a[0]) and np.array_equal(b[2], -a[2]) and np.array_equal(b[1], a[1])
    mirrored = a[:, ::-1, ::-1]
    assert np.array_equal(mirrored[0], -a[0]) and np.array_equal(mirrored[2], -a[2]) and np.array_equal(mirrored[1], a[1])
    assert np.array_equal(b, mirrored)
    # the pose takes camera coordinates to point-cloud coordinates: a camera turned a quarter about y looks along +x of the scene
    quarter = np.array([0, np.sqrt(0.5), 0, np.sqrt(0.5)], dtype=np.float32)
    centre = ref.colours(coef, 1, quarter, ref.camera(1, 1, cx=0.5, cy=0.5), 1, 1)      # the one pixel is the optical axis
    assert abs(centre[2, 0, 0] - np.float32(-0.48860251190291987)) < 1e-6 and abs(centre[1, 0, 0]) < 1e-6


def test_the_sums_follow_the_headers_order():
    """1 + 2^-24 in f32 is 1: the two small terms of one thread are added first only if they come first"""
    t = np.float32(2.0 ** -24)
    terms = np.zeros(2048, dtype=np.float32)
    sel = np.ones(2048, dtype=bool)
    terms[0], terms[1], terms[2] = 1.0, t, t              # one thread, ascending: (1 + t) + t = 1
    assert ref.block_sums(terms, sel)[0] == np.float32(1.0)
    terms[:3] = t, t, 1.0                                 # (t + t) + 1 keeps the bit
    assert ref.block_sums(terms, sel)[0] == np.float32(1.0) + np.float32(2.0 ** -23)
    terms[:] = 0.0
    terms[0], terms[4 * 32] = 1.0, t                      # lanes 0 and 32 meet in the first butterfly step
    terms[4], terms[4 * 33] = t, 0.0
    assert ref.block_sums(terms, sel)[0] == np.float32(1.0)
    # the finishing sum is float64 and rounds once: 257 blocks, thread 0 takes blocks 0 and 256
    partial = np.full(257, t, dtype=np.float32)
    partial[0] = 1.0
    assert ref.finish(partial) == np.float32(1.0 + 256 * 2.0 ** -24)
    sel[:] = False
    assert np.all(ref.block_sums(np.full(2048, np.nan, dtype=np.float32), sel) == 0.0)


def test_selection_keeps_nan_out_of_every_sum():
    x, A, g, coef, q, K9 = _case(40)
    clean = ref.grad_coef(g, A, 3, q, K9)
    g[:, 1, 1] = 0.0
    g[:, 4, 2] = [0.0, -0.0, 0.0]
    base = ref.grad_coef(g, A, 3, q, K9)
    A[1, 1], A[4, 2] = np.nan, np.inf
    assert ref.grad_coef(g, A, 3, q, K9).tobytes() == base.tobytes() and base.tobytes() != clean.tobytes()
    ga = ref.grad_alpha(g, coef, 3, q, K9)
    assert ga[1, 1] == 0.0 and ga[4, 2] == 0.0 and not np.signbit(ga[4, 2]) and np.all(np.isfinite(ga))
    g[1, 5, 5] = np.nan                                   # a NaN upstream is selected and shows
    assert np.isnan(ref.grad_alpha(g, coef, 3, q, K9)[5, 5]) and np.all(np.isnan(ref.grad_coef(g, A, 3, q, K9)[16:32]))
