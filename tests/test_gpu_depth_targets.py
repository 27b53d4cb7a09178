"""GPU (-m gpu): gs_depth_resample (include/gs_depth.h), through depth.depth_resample and DepthStore, against its float64
restatement (tests/depth_ref.resample).

Sources: 70x150 uint16 with a row pitch that is no multiple of 16 (nor of 4); 130x200, whose factor-1 crop is 128x192 -- three
64-wide and eight 16-row tiles; an f32 source whose holes are NaN, inf, 0 and negative values; 50 rows to 16, a non-integer
scale.  Holes: a single sample, a block, a whole row, every sample, and a lattice that leaves no filter window whole.

Bars: at factor 1 both planes are bit-exact.  Elsewhere the weight is within the resampler's 2e-6 (tests/test_gpu_targets.py) of
the reference, and the depth within (2 * 2e-6 * z_max) / den_ref plus one f32 ulp of the value: the filter's bar on numerator
and denominator, carried through the quotient.  A pixel whose den_ref is within 1e-5 of min_coverage may fall on either side
of the threshold and is left out (not one whose den_ref is exactly 0: no valid sample, exactly 0 on the device); every case asserts on the CPU that this leaves out at most 0.1 % of its pixels (0.3 and 0.55
are no multiples of 1/64, the lattice of the factor-2 weights; min_coverage = 1 is tested where no window is nearly whole)."""
import functools

import numpy as np
import pytest
import torch

import depth_ref as R
from taichi_3d_gaussian_splatting_amd import depth, targets
from test_gpu_targets import GUARD_BITS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ABS_TOL = 2e-6
NEAR_THRESHOLD = 1e-5
MAX_EXCLUDED = 0.001
SCALE = 0.001


@functools.lru_cache(maxsize=None)
def u16_map(H, W, holes, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    d = (2000 + 40 * x + 25 * y + rng.integers(0, 3000, (H, W))).astype(np.uint16)
    assert d.min() > 0
    if holes == "some":
        d[5, 7] = 0                                        # a single sample
        d[20:31, 40:63] = 0                                # a block
        d[H // 2 + 3, :] = 0                               # a whole row
        d[rng.random((H, W)) < 0.03] = 0
    elif holes == "all":
        d[:] = 0
    elif holes == "lattice":                               # every second row and column: no window of two or more taps is whole
        d[::2, :] = 0
        d[:, ::2] = 0
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def f32_map(H, W, holes, seed=0):
    u = u16_map(H, W, "none", seed)
    z = (u.astype(np.float32) * np.float32(SCALE)).copy()
    bad = np.array([np.nan, np.inf, -np.inf, 0.0, -1.5, -0.0], np.float32)
    if holes == "some":
        mask = u16_map(H, W, "some", seed) == 0
        z[mask] = bad[np.arange(mask.sum()) % len(bad)]
    elif holes == "all":
        z[:] = bad[np.arange(H * W) % len(bad)].reshape(H, W)
    z.setflags(write=False)
    return z


def on_device(array, pitch_elems=None):
    """the map on the device; uint16 with the given row pitch in samples (default: dense) inside a buffer of non-zero filler"""
    if array.dtype != np.uint16:
        return torch.from_numpy(np.array(array)).to(DEV)
    H, W = array.shape
    pitch = W if pitch_elems is None else pitch_elems
    host = np.full(H * pitch + 32, 0xA5A5, np.uint16)
    rows = np.lib.stride_tricks.as_strided(host, (H, W), (2 * pitch, 2))
    rows[:] = array
    return torch.from_numpy(host).to(DEV).as_strided((H, W), (pitch, 1))


def run(src, size_full, crop, depth_scale, min_coverage):
    """-> the (2,h,w) result, after checking the words around it and that a second run gives the same bits"""
    h, w = crop
    guard = 2 * w + 4
    guard += (-guard) % 4
    buf = torch.full((guard + 2 * h * w + guard,), GUARD_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
    out = buf[guard:guard + 2 * h * w].view(2, h, w)
    got = depth.depth_resample(src, size_full, crop, depth_scale=depth_scale, min_coverage=min_coverage, out=out)
    assert got.data_ptr() == out.data_ptr()
    again = depth.depth_resample(src, size_full, crop, depth_scale=depth_scale, min_coverage=min_coverage)
    torch.cuda.synchronize()
    words = buf.view(torch.int32)
    assert bool((words[:guard] == GUARD_BITS).all()) and bool((words[guard + 2 * h * w:] == GUARD_BITS).all()), "the kernel wrote outside its output"
    assert torch.equal(out.view(torch.int32), again.view(torch.int32)), "two runs differ"
    return out.cpu().numpy()


def check(array, fmt, size_full, crop, min_coverage, pitch_elems=None, identity=False):
    want_depth, want_weight, den = R.resample(array, fmt, size_full, crop, SCALE, min_coverage)
    got = run(on_device(array, pitch_elems), size_full, crop, SCALE if fmt == R.FORMAT_U16 else 1.0, min_coverage)
    assert np.isfinite(got).all()
    assert not np.signbit(got).any()                       # an empty pixel is +0 in both planes
    if identity:
        assert np.array_equal(got[0].astype(np.float64), want_depth) and np.array_equal(got[1].astype(np.float64), want_weight)
        return
    # (a den_ref of exactly 0 is a window without a valid sample: exactly 0 on the device too, and not left out)
    near = (np.abs(den - min_coverage) < NEAR_THRESHOLD) & (den > 0)
    assert near.mean() <= MAX_EXCLUDED, f"{near.mean():.4%} of the pixels sit on the threshold: choose other inputs"
    keep = ~near
    err_w = np.abs(got[1] - want_weight)[keep]
    z_max = float(R.samples(array, fmt, SCALE)[1].max())
    bar = 2 * ABS_TOL * z_max / np.where(den > 0, den, 1.0) + np.spacing(np.abs(want_depth).astype(np.float32)).astype(np.float64)
    err_d = np.abs(got[0] - want_depth)
    print(f"weight max error {err_w.max() if err_w.size else 0:.3g}; depth max error / bar {(err_d / bar)[keep].max() if keep.any() else 0:.3g}; "
          f"left out {int(near.sum())}")
    assert err_w.size == 0 or err_w.max() <= ABS_TOL
    assert np.all((err_d <= bar)[keep])
    assert np.all((got[0] == 0) == (got[1] == 0)), "a depth without a weight, or a weight without a depth"


COVERAGES = [0.0, 0.3, 0.55]


@pytest.mark.parametrize("min_coverage", COVERAGES + [1.0])
@pytest.mark.parametrize("fmt", [R.FORMAT_U16, R.FORMAT_F32], ids=["u16", "f32"])
def test_factor_one_is_the_identity(fmt, min_coverage):
    # 70x150 -> its 64x144 crop (pitch 153 samples: rows at 2-byte alignment only); 130x200 -> 128x192, 3 x 8 tiles
    a = u16_map(70, 150, "some") if fmt == R.FORMAT_U16 else f32_map(70, 150, "some")
    check(a, fmt, (70, 150), (64, 144), min_coverage, pitch_elems=153, identity=True)
    b = u16_map(130, 200, "some", seed=1) if fmt == R.FORMAT_U16 else f32_map(130, 200, "some", seed=1)
    assert targets.downsampled_geometry(130, 200, 1) == (130, 200, 128, 192)
    check(b, fmt, (130, 200), (128, 192), min_coverage, pitch_elems=208, identity=True)


@pytest.mark.parametrize("min_coverage", COVERAGES)
@pytest.mark.parametrize("fmt", [R.FORMAT_U16, R.FORMAT_F32], ids=["u16", "f32"])
def test_factor_two(fmt, min_coverage):
    a = u16_map(70, 150, "some") if fmt == R.FORMAT_U16 else f32_map(70, 150, "some")
    assert targets.downsampled_geometry(70, 150, 2) == (35, 75, 32, 64)
    check(a, fmt, (35, 75), (32, 64), min_coverage, pitch_elems=153)
    b = u16_map(130, 200, "some", seed=1) if fmt == R.FORMAT_U16 else f32_map(130, 200, "some", seed=1)
    check(b, fmt, (65, 100), (64, 96), min_coverage, pitch_elems=208)


@pytest.mark.parametrize("min_coverage", COVERAGES)
@pytest.mark.parametrize("fmt", [R.FORMAT_U16, R.FORMAT_F32], ids=["u16", "f32"])
def test_non_integer_scale(fmt, min_coverage):
    a = u16_map(50, 101, "some", seed=2) if fmt == R.FORMAT_U16 else f32_map(50, 101, "some", seed=2)
    check(a, fmt, (16, 40), (16, 37), min_coverage, pitch_elems=103)         # 37 columns: no 16-byte store


@pytest.mark.parametrize("size_full,crop", [((70, 150), (64, 144)), ((35, 75), (32, 64)), ((23, 50), (16, 48))])
def test_an_all_invalid_map_gives_zeros(size_full, crop):
    for array, fmt in ((u16_map(70, 150, "all"), R.FORMAT_U16), (f32_map(70, 150, "all"), R.FORMAT_F32)):
        for min_coverage in (0.0, 1.0):
            got = run(on_device(array, 153), size_full, crop, SCALE, min_coverage)
            assert not got.any() and not np.signbit(got).any()


@pytest.mark.parametrize("size_full,crop", [((35, 75), (32, 64)), ((23, 50), (16, 48))])
def test_full_coverage_drops_every_window_with_a_hole(size_full, crop):
    """min_coverage = 1 where no window is whole: every weight is 0; at min_coverage 0 the same map is the mean of what is valid"""
    array = u16_map(70, 150, "lattice")
    _, _, den = R.resample(array, R.FORMAT_U16, size_full, crop, SCALE, 1.0)
    assert den.max() < 1.0 - 0.1
    check(array, R.FORMAT_U16, size_full, crop, 1.0, pitch_elems=153)
    check(array, R.FORMAT_U16, size_full, crop, 0.0, pitch_elems=153)


def test_a_hole_reaches_nothing():
    """whatever an invalid f32 sample holds, the result is the same bits"""
    a = np.array(f32_map(70, 150, "some"))
    with np.errstate(invalid="ignore"):
        holes = ~(np.isfinite(a) & (a > 0))
    b = a.copy()
    b[holes] = np.float32(-7.0)
    c = a.copy()
    c[holes] = np.float32(np.nan)
    outs = [run(on_device(v), (35, 75), (32, 64), 1.0, 0.3) for v in (a, b, c)]
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


def test_depth_store_hands_out_both_planes_of_one_buffer():
    class _Dataset:
        maps = [(np.array(u16_map(70, 150, "some")), 0.002), (np.array(f32_map(70, 150, "some")), None), None]

        def __len__(self):
            return len(self.maps)

        def load_depth(self, i):
            return self.maps[i]

    with pytest.raises(ValueError, match="depth_path"):
        depth.DepthStore.from_dataset(_Dataset(), DEV)
    store = depth.DepthStore.from_dataset(_Dataset(), DEV, require_all=False)
    assert [store.has(i) for i in range(3)] == [True, True, False]
    assert store.maps[0].dtype == torch.uint16 and (store.maps[0].stride(0) * 2) % 16 == 0 and store.maps[1].dtype == torch.float32
    for f in (1, 2):
        h_full, w_full, h, w = targets.downsampled_geometry(64, 144, f)
        z, wt = store.target(0, f, 0.3)
        assert z.shape == wt.shape == (h, w) and z.is_contiguous() and wt.is_contiguous()
        assert wt.data_ptr() == z.data_ptr() + 4 * h * w
        want = depth.depth_resample(on_device(np.array(u16_map(70, 150, "some")[:64, :144])), (h_full, w_full), (h, w), depth_scale=0.002, min_coverage=0.3)
        assert torch.equal(z, want[0]) and torch.equal(wt, want[1])
        first = z.data_ptr()
        allocated = torch.cuda.memory_allocated()
        z1, _ = store.target(1, f, 0.3)
        assert z1.data_ptr() == first and torch.cuda.memory_allocated() == allocated        # the same buffer, nothing new
        want = depth.depth_resample(on_device(np.array(f32_map(70, 150, "some")[:64, :144])), (h_full, w_full), (h, w), min_coverage=0.3)
        assert torch.equal(z1, want[0])
    with pytest.raises(ValueError, match="no depth map"):
        store.target(2, 1)
