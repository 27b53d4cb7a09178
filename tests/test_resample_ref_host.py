"""CPU: the float64 numpy restatement of the antialiased resize (tests/resample_ref.py) against torch's own operator in
float64, at integer and non-integer scales, one axis untouched, and equal sizes."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resample_ref

PAIRS = [((64, 96), (16, 24)), ((64, 96), (32, 48)), ((37, 53), (9, 13)), ((135, 240), (128, 200)), ((50, 70), (12, 17)),
         ((33, 47), (33, 20)), ((48, 80), (48, 80))]


def _image(shape, seed=0):
    return np.random.default_rng(seed).uniform(0.0, 1.0, (3, *shape))


@pytest.mark.parametrize("src,dst", PAIRS, ids=lambda p: "x".join(map(str, p)))
def test_matches_interpolate_antialias_in_float64(src, dst):
    image = _image(src)
    want = F.interpolate(torch.tensor(image, dtype=torch.float64)[None], size=dst, mode="bilinear", antialias=True,
                         align_corners=False)[0].numpy()
    got = resample_ref.resize_antialias(image, dst)
    assert got.shape == want.shape == (3, *dst)
    assert np.abs(got - want).max() <= 1e-12


def test_equal_sizes_are_the_identity_exactly():
    image = _image((48, 80), seed=1)
    assert np.array_equal(resample_ref.resize_antialias(image, (48, 80)), image)


def test_crop_is_the_top_left_of_the_full_resize():
    image = _image((80, 112), seed=2)
    full = resample_ref.resize_antialias(image, (40, 56))
    assert np.array_equal(resample_ref.resize_antialias(image, (40, 56), (32, 48)), full[:, :32, :48])


def test_windows_have_at_most_two_scale_plus_one_taps_and_weights_sum_to_one():
    for n_in, n_out in [(96, 24), (240, 200), (128, 16), (53, 13)]:
        for lo, w in resample_ref.axis_windows(n_in, n_out):
            assert 1 <= len(w) <= 2 * n_in / n_out + 1 and lo >= 0 and lo + len(w) <= n_in
            assert abs(w.sum() - 1.0) < 1e-15


def test_target_geometry_is_the_trainers():
    u8 = np.random.default_rng(3).integers(0, 256, (80, 112, 4), dtype=np.uint8)
    assert resample_ref.target(u8, 2).shape == (3, 32, 48)
    assert resample_ref.target(u8, 1).shape == (3, 80, 112)
    assert np.array_equal(resample_ref.target(u8, 1), resample_ref.to_float(u8))
