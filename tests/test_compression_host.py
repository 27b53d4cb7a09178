"""CPU: the codec of compressed scene files (compression.py: encode, decode, save, load) on host arrays."""
import numpy as np
import pytest
import torch

from taichi_3d_gaussian_splatting_amd import compression

REST = list(range(9, 24)) + list(range(25, 40)) + list(range(41, 56))


def _scene(n=300, k=40, seed=0):
    rng = np.random.default_rng(seed)
    pc = rng.normal(0, 3, (n, 3)).astype(np.float32)
    ft = rng.normal(0, 1, (n, 56)).astype(np.float32)
    ft[:, 0:4] *= 1.7                                               # not unit quaternions
    codebook = rng.normal(0, 0.3, (k, 45)).astype(np.float32)
    index = rng.integers(0, k, n).astype(np.int32)
    index[:2] = [0, k - 1]
    return pc, ft, index, codebook


def test_columns_dtypes_and_the_index_width():
    pc, ft, index, codebook = _scene()
    c = compression.encode(pc, ft, index, codebook)
    assert compression.REST_COLUMNS == tuple(REST) and compression.DC_COLUMNS == (8, 24, 40) and compression.FORMAT == "gsvq1"
    assert c.xyz.dtype == np.float32 and np.array_equal(c.xyz, pc)
    for name, cols in (("q", [0, 1, 2, 3]), ("log_scale", [4, 5, 6]), ("sh_dc", [8, 24, 40])):
        a = getattr(c, name)
        assert a.dtype == np.float16 and np.array_equal(a, ft[:, cols].astype(np.float16))
    assert c.opacity_logit.dtype == np.float16 and np.array_equal(c.opacity_logit, ft[:, 7].astype(np.float16))
    assert c.codebook.dtype == np.float16 and c.codebook.shape == (40, 45) and c.sh_index.dtype == np.uint8
    assert c.nbytes() == 300 * compression.BYTES_PER_GAUSSIAN - 300 + 40 * 90 and compression.BYTES_PER_GAUSSIAN == 36
    for k, dtype in ((256, np.uint8), (257, np.uint16), (65536, np.uint16)):
        pc, ft, index, codebook = _scene(n=20, k=k)
        assert compression.encode(pc, ft, index, codebook).sh_index.dtype == dtype
    pc2, ft2 = c.decode()
    pc, ft, index, codebook = _scene()
    assert pc2.dtype == ft2.dtype == torch.float32 and tuple(ft2.shape) == (300, 56) and np.array_equal(pc2.numpy(), pc)
    # every decoded SH row is its codebook row, channel-major: R1..R15, G1..G15, B1..B15
    assert np.array_equal(ft2.numpy()[:, REST], c.codebook.astype(np.float32)[index])
    assert np.array_equal(ft2.numpy()[:, 9:24], codebook[index][:, 0:15].astype(np.float16).astype(np.float32))
    assert np.array_equal(ft2.numpy()[:, 41:56], codebook[index][:, 30:45].astype(np.float16).astype(np.float32))


def test_half_precision_bound_clamp_and_the_quaternion_as_stored():
    pc, ft, index, codebook = _scene()
    ft[0, 4], ft[1, 4], ft[2, 7], ft[3, 8] = 1e6, -1e6, np.inf, np.nan
    c = compression.encode(pc, ft, index, codebook)
    assert c.log_scale[0, 0] == np.float16(65504) and c.log_scale[1, 0] == np.float16(-65504) and c.opacity_logit[2] == np.float16(65504)
    assert np.isnan(c.sh_dc[3, 0])
    _, got = c.decode()
    got = got.numpy()
    cols = [0, 1, 2, 3, 4, 5, 6, 7, 8, 24, 40]
    x = ft[4:, cols].astype(np.float64)
    normal = np.abs(x) >= 2.0 ** -14                                # f16's normal range: relative error 2^-11
    assert normal.mean() > 0.99
    assert np.all(np.abs(got[4:, cols].astype(np.float64) - x)[normal] <= 2.0 ** -11 * np.abs(x)[normal])
    assert np.all(np.abs(got[4:, cols].astype(np.float64) - x)[~normal] <= 2.0 ** -25)
    norms = np.linalg.norm(got[4:, 0:4], axis=1)
    assert np.all(np.abs(norms - np.linalg.norm(ft[4:, 0:4], axis=1)) < 0.01) and np.abs(norms - 1.0).max() > 0.5   # not normalised
    assert np.array_equal(compression.to_f16(torch.tensor([0.1, 65520.0, -1e9, 2049.0, 2051.0])),
                          np.array([0.1, 65504, -65504, 2048, 2052], np.float16))        # ties go to even


def test_file_round_trip_and_format_check(tmp_path):
    pc, ft, index, codebook = _scene(n=500, k=300)
    c = compression.encode(pc, ft, index, codebook)
    path = tmp_path / "scene.npz"
    c.save(path)
    with np.load(path) as z:
        assert sorted(z.files) == sorted(compression.KEYS) and str(z["format"]) == "gsvq1"
        assert z["sh_index"].dtype == np.uint16 and z["codebook"].shape == (300, 45)
    back = compression.load(path)
    for name in compression.KEYS[1:]:
        assert np.array_equal(getattr(back, name), getattr(c, name), equal_nan=True), name
    a, b = c.decode(), back.decode()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    other = tmp_path / "other.npz"
    np.savez_compressed(other, format=np.array("gsvq0"), **{k: getattr(c, k) for k in compression.KEYS[1:]})
    with pytest.raises(ValueError, match="gsvq1"):
        compression.load(other)
    np.savez_compressed(other, xyz=c.xyz)
    with pytest.raises(ValueError, match="gsvq1"):
        compression.load(other)


def test_rows_without_a_codebook_entry_are_refused():
    pc, ft, index, codebook = _scene()
    index[5] = -1
    with pytest.raises(ValueError, match="label -1"):
        compression.encode(pc, ft, index, codebook)
    index[5] = 40
    with pytest.raises(ValueError):
        compression.encode(pc, ft, index, codebook)
